"""NV12 video frames: the container, the conversion rule, and the numpy restatements that define the HIP kernels
lp_nv12_to_bgr_batch and lp_preprocess_nv12_batch (csrc/lp_nv12.hip) bit for bit.

A frame is h x w with h and w even.  Its planes:
  y  uint8 [h, w]        rows ``pitch_y`` >= w bytes apart;
  uv uint8 [h/2, w/2, 2] U first, rows ``pitch_uv`` >= w bytes apart (even), base 2-byte aligned.
Pixel (i, j) takes Y = y[i][j], U = uv[i >> 1][j >> 1][0], V = uv[i >> 1][j >> 1][1]: chroma is replicated, not
interpolated (what OpenCV's NV12 conversion does).  In int32, with an arithmetic right shift:

    c = max(Y - yoff, 0) * CY;  d = U - 128;  e = V - 128;  half = 1 << 19
    R = clamp255((c + half + CVR*e) >> 20)
    G = clamp255((c + half + CVG*e + CUG*d) >> 20)
    B = clamp255((c + half + CUB*d) >> 20)

``MATRICES`` holds (id, yoff, CY, CUB, CUG, CVG, CVR) of the four supported matrices; these integers are the specification.
'bt601' is the table of OpenCV's COLOR_YUV2BGR_NV12 (made from 3-decimal constants; its equality with cv2.cvtColor is not
checked anywhere here: OpenCV is not a dependency).  The other three are round(x * 2^20) of the standards' matrices.
Over all 2^24 (Y, U, V) the largest accumulator magnitude is below 5.9e8, so int32 is enough.
"""
import numpy as np

try:
    import torch
except ImportError:        # the numpy half of this module works without it
    torch = None

#: name -> (id, yoff, CY, CUB, CUG, CVG, CVR)
MATRICES = {
    'bt601': (0, 16, 1220542, 2116026, -409993, -852492, 1673527),      # limited range
    'bt709': (1, 16, 1220945, 2215014, -223607, -558796, 1879825),      # limited range
    'bt601f': (2, 0, 1048576, 1858077, -360853, -748826, 1470104),      # full range
    'bt709f': (3, 0, 1048576, 1945738, -196424, -490864, 1651297),      # full range
}
MATRIX_NAMES = tuple(sorted(MATRICES, key=lambda k: MATRICES[k][0]))
SHIFT = 20


def _is_tensor(a):
    return torch is not None and torch.is_tensor(a)


def _strides_bytes(a):
    """Byte strides of a uint8 numpy array or torch tensor."""
    return tuple(int(s) for s in (a.stride() if _is_tensor(a) else a.strides))


class Nv12Frame:
    """One NV12 frame: ``y`` uint8 [h, w] and ``uv`` uint8 [h/2, w/2, 2] (numpy arrays, or torch tensors on one device), either
    possibly a view with a row pitch above its width, and the name of its matrix.  ``shape`` is (h, w, 3), the shape of
    the BGR frame it stands for, so the geometry helpers written for BGR frames take it as it is."""

    def __init__(self, y, uv, matrix='bt601'):
        if matrix not in MATRICES:
            raise ValueError('unknown NV12 matrix %r (one of %s)' % (matrix, ', '.join(MATRIX_NAMES)))
        if _is_tensor(y) != _is_tensor(uv):
            raise ValueError('y and uv must both be numpy arrays or both be torch tensors')
        u8 = torch.uint8 if _is_tensor(y) else np.uint8
        if y.dtype != u8 or uv.dtype != u8 or len(y.shape) != 2 or len(uv.shape) != 3:
            raise ValueError('NV12 planes must be uint8 y [h, w] and uv [h/2, w/2, 2]')
        h, w = int(y.shape[0]), int(y.shape[1])
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError('NV12 frames need even sizes, got %d x %d' % (h, w))
        if tuple(uv.shape) != (h // 2, w // 2, 2):
            raise ValueError('uv must be [%d, %d, 2] for a %d x %d frame, got %s' % (h // 2, w // 2, h, w, list(uv.shape)))
        sy, suv = _strides_bytes(y), _strides_bytes(uv)
        if sy[1] != 1 or sy[0] < w:
            raise ValueError('y rows must be contiguous and at least w bytes apart')
        if suv[2] != 1 or suv[1] != 2 or suv[0] < w or suv[0] % 2:
            raise ValueError('uv rows must hold interleaved U, V pairs and be an even number of bytes >= w apart')
        if _is_tensor(y):
            if y.device != uv.device:
                raise ValueError('y and uv must be on one device')
            if uv.data_ptr() % 2:
                raise ValueError('uv must be 2-byte aligned')
        self.y, self.uv, self.matrix = y, uv, matrix
        self.h, self.w = h, w
        self.pitch_y, self.pitch_uv = sy[0], suv[0]

    @property
    def shape(self):
        return (self.h, self.w, 3)

    @property
    def matrix_id(self):
        return MATRICES[self.matrix][0]

    @property
    def is_tensor(self):
        return _is_tensor(self.y)

    @property
    def is_cuda(self):
        return self.is_tensor and self.y.is_cuda

    @property
    def device(self):
        return self.y.device if self.is_tensor else None

    @property
    def nbytes(self):
        """Bytes of a packed frame of this size (h * w * 3 / 2)."""
        return self.h * self.w * 3 // 2

    @classmethod
    def from_packed(cls, buf, h, w, matrix='bt601'):
        """Views of one contiguous packed frame ``buf`` (h * 3 / 2 rows of w bytes: the Y plane, then the UV plane; any
        shape with that many elements): nothing is copied."""
        h, w = int(h), int(w)
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError('NV12 frames need even sizes, got %d x %d' % (h, w))
        n = h * w * 3 // 2
        if _is_tensor(buf):
            if buf.numel() != n or not buf.is_contiguous():
                raise ValueError('a packed %d x %d NV12 frame is %d contiguous bytes' % (h, w, n))
            flat = buf.view(-1)
            return cls(flat[:h * w].view(h, w), flat[h * w:].view(h // 2, w // 2, 2), matrix)
        if buf.size != n or not buf.flags['C_CONTIGUOUS']:
            raise ValueError('a packed %d x %d NV12 frame is %d contiguous bytes' % (h, w, n))
        flat = buf.reshape(-1)
        return cls(flat[:h * w].reshape(h, w), flat[h * w:].reshape(h // 2, w // 2, 2), matrix)

    def packed(self):
        """A new contiguous uint8 numpy array [h * 3 / 2, w] of a host frame (Y rows, then UV rows)."""
        out = np.empty((self.h * 3 // 2, self.w), np.uint8)
        out[:self.h] = _host(self.y)
        out[self.h:] = _host(self.uv).reshape(self.h // 2, self.w)
        return out

    def to(self, device):
        """The frame with both planes copied to a torch device (packed: pitches become w)."""
        buf = torch.from_numpy(self.packed()).to(device)
        return Nv12Frame.from_packed(buf, self.h, self.w, self.matrix)


def _host(a):
    return a.cpu().numpy() if _is_tensor(a) else np.asarray(a)


def is_nv12_list(frames, what='frames'):
    """True when every element of ``frames`` is an ``Nv12Frame``, False when none is; a mixed list is a ValueError."""
    kinds = set(isinstance(f, Nv12Frame) for f in frames if f is not None)
    if len(kinds) > 1:
        raise ValueError('%s mix NV12 and BGR frames: one call takes one kind' % what)
    return kinds == {True}


def yuv_to_bgr_np(Y, U, V, matrix):
    """The rule on int arrays of one shape: uint8 array [..., 3] in B, G, R order."""
    _, yoff, CY, CUB, CUG, CVG, CVR = MATRICES[matrix]
    c = np.maximum(Y.astype(np.int32) - yoff, 0) * np.int32(CY) + np.int32(1 << (SHIFT - 1))
    d = U.astype(np.int32) - 128
    e = V.astype(np.int32) - 128
    out = np.empty(c.shape + (3,), np.uint8)
    out[..., 0] = np.clip((c + CUB * d) >> SHIFT, 0, 255)
    out[..., 1] = np.clip((c + CVG * e + CUG * d) >> SHIFT, 0, 255)
    out[..., 2] = np.clip((c + CVR * e) >> SHIFT, 0, 255)
    return out


def nv12_to_bgr_np(frame):
    """uint8 [h, w, 3] BGR of an ``Nv12Frame`` by the rule in the module's docstring."""
    y, uv = _host(frame.y), _host(frame.uv)
    u = np.repeat(np.repeat(uv[:, :, 0], 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(uv[:, :, 1], 2, axis=0), 2, axis=1)
    return yuv_to_bgr_np(y, u, v, frame.matrix)


def float_matrix(matrix):
    """(yoff, M): the float64 form of the rule, [B, G, R] = M @ [Y - yoff, U - 128, V - 128] before rounding and clipping."""
    _, yoff, CY, CUB, CUG, CVG, CVR = MATRICES[matrix]
    M = np.array([[CY, CUB, 0], [CY, CUG, CVG], [CY, 0, CVR]], np.float64) / float(1 << SHIFT)
    return yoff, M


def bgr_to_nv12_np(bgr, matrix='bt601'):
    """Host encoder (a stand-in for a decoder's output: it makes inputs for tests, the benchmarks and ``--nv12``): the inverse
    of the matrix in float64; Y per pixel, U and V the mean over each 2 x 2 block; all rounded half up and clipped to 0..255.
    Odd sizes are rejected.  Returns a packed host ``Nv12Frame``."""
    if matrix not in MATRICES:
        raise ValueError('unknown NV12 matrix %r (one of %s)' % (matrix, ', '.join(MATRIX_NAMES)))
    bgr = np.asarray(bgr)
    if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError('bgr must be a uint8 [h, w, 3] array, got %s %s' % (bgr.dtype, bgr.shape))
    h, w = bgr.shape[:2]
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError('NV12 frames need even sizes, got %d x %d' % (h, w))
    yoff, M = float_matrix(matrix)
    yuv = bgr.astype(np.float64) @ np.linalg.inv(M).T                   # [h, w, 3] = Y - yoff, U - 128, V - 128
    buf = np.empty((h * 3 // 2, w), np.uint8)
    buf[:h] = np.clip(np.floor(yuv[:, :, 0] + yoff + 0.5), 0, 255)
    chroma = yuv[:, :, 1:].reshape(h // 2, 2, w // 2, 2, 2).mean(axis=(1, 3)) + 128.0
    buf[h:] = np.clip(np.floor(chroma + 0.5), 0, 255).reshape(h // 2, w)
    return Nv12Frame.from_packed(buf, h, w, matrix)


def _network_input(img_bgr_u8):
    """letterboxed uint8 [H, W, 3] BGR -> float32 [3, H, W] RGB, v / 255 in fp32: the kernels' value before the cast to the
    output dtype (round to nearest even)."""
    return np.ascontiguousarray(img_bgr_u8.transpose(2, 0, 1)[::-1]).astype(np.float32) / np.float32(255)


def letterbox_nv12_np(frame, img_size, stride=32, auto=True):
    """The definition of the fused letterbox on a whole frame: convert the whole frame (``nv12_to_bgr_np``), then the BGR
    path's restatement (``data_augment.letterbox`` with the fixed-point resize, BGR -> RGB, / 255).  float32 [3, H, W]."""
    from yolov6.data.data_augment import resize_linear_u8, letterbox_geometry
    return _letterbox_bgr(nv12_to_bgr_np(frame), img_size, stride, auto, letterbox_geometry, resize_linear_u8)


def region_nv12_np(frame, y0, x0, th, tw, img_size, stride=32):
    """The definition of the fused letterbox on a region: convert the whole frame, copy the region
    [y0:y0+th, x0:x0+tw] of it, and letterbox the copy to exactly ``img_size`` (``auto=False``): the bilinear taps clamp at
    the region's edges, the chroma of a pixel is that of its absolute frame coordinate.  float32 [3, H, W]."""
    from yolov6.data.data_augment import resize_linear_u8, letterbox_geometry
    if not (0 <= y0 and 0 <= x0 and th >= 1 and tw >= 1 and y0 + th <= frame.h and x0 + tw <= frame.w):
        raise ValueError('region (%d, %d, %d, %d) is not inside the %d x %d frame' % (y0, x0, th, tw, frame.h, frame.w))
    region = np.ascontiguousarray(nv12_to_bgr_np(frame)[y0:y0 + th, x0:x0 + tw])
    return _letterbox_bgr(region, img_size, stride, False, letterbox_geometry, resize_linear_u8)


def _letterbox_bgr(bgr, img_size, stride, auto, letterbox_geometry, resize_linear_u8):
    size = list(img_size) if isinstance(img_size, (list, tuple)) else int(img_size)
    _, (rw, rh), (top, bottom, left, right), _ = letterbox_geometry(bgr.shape[:2], size, auto=auto, stride=stride)
    if (rh, rw) != bgr.shape[:2]:
        bgr = resize_linear_u8(bgr, (rw, rh))                          # always the fixed-point scheme the kernels restate
    out = np.full((rh + top + bottom, rw + left + right, 3), 114, np.uint8)
    out[top:top + rh, left:left + rw] = bgr
    return _network_input(out)


def read_nv12_stream(path, h, w, matrix='bt601', batch=1):
    """Read a raw stream of packed NV12 frames (h * 3 / 2 * w bytes each) with ``np.fromfile``, ``batch`` frames at a time:
    yields lists of host ``Nv12Frame`` views (the last list may be shorter; trailing bytes short of a frame are an error)."""
    import os
    h, w, batch = int(h), int(w), int(batch)
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError('NV12 frames need even sizes, got %d x %d' % (h, w))
    if batch < 1:
        raise ValueError('batch must be >= 1')
    n = h * w * 3 // 2
    size = os.path.getsize(path)
    if size % n:
        raise ValueError('%s: %d bytes is not a whole number of %d x %d NV12 frames (%d bytes each)' % (path, size, w, h, n))
    total = size // n
    for k in range(0, total, batch):
        count = min(batch, total - k)
        buf = np.fromfile(path, dtype=np.uint8, count=count * n, offset=k * n).reshape(count, h * 3 // 2, w)
        yield [Nv12Frame.from_packed(buf[j], h, w, matrix) for j in range(count)]
