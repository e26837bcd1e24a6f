"""What the modules of the host runtime share: the dtype tables, pointers for the C ABI, per-stream workspaces and persistent
buffers, the checks of frame lists and padded detections, and the descriptor arrays and runs of frames that the per-frame
launches (redaction, overlay, JPEG) are made of."""
import ctypes

import torch

from yolov6.hip import abi
from yolov6.utils.nv12 import Nv12Frame, is_nv12_list

_DT = {torch.float16: abi.LP_F16, torch.bfloat16: abi.LP_BF16, torch.float32: abi.LP_F32}
_TORCH_DT = {v: k for k, v in _DT.items()}


def _dptr(t):
    """Device pointer of a tensor for the C ABI (None stays a null pointer)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _aligned(buf):
    """256-byte aligned base address inside ``buf``: arenas and workspaces are allocated 256 bytes larger than needed."""
    return (buf.data_ptr() + 255) // 256 * 256


def _stream_ptr(device):
    """torch's current stream on ``device`` as the hipStream_t every launch of the library goes to."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _aligned_span(ws):
    """(aligned base as a pointer, bytes from it to the end) of a workspace whose launch takes all that is there."""
    base = _aligned(ws)
    return ctypes.c_void_p(base), ws.numel() - (base - ws.data_ptr())


def _cuda_device(device, what):
    """The indexed CUDA device of a ``device`` argument (a bare 'cuda' is the current device); ValueError(``what``) for any other kind."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ValueError(what)
    return torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)


def _stream_workspace(cache, device, need):
    """``cache``'s workspace of ``device``'s current stream, grown to ``need`` bytes (+ 256 for ``_aligned``), never zeroed."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < need + 256:
        ws = cache[key] = torch.empty(need + 256, dtype=torch.uint8, device=device)
    return ws


def _persistent(cache, key, make):
    """``cache[key]``, from ``make()`` at the first use of the key: the persistent buffers of one call shape."""
    buf = cache.get(key)
    if buf is None:
        buf = cache[key] = make()
    return buf


def _buffer(buf, shape, dtype, device, what='out'):
    """A caller's persistent output buffer, checked; a new tensor of that ``shape`` / ``dtype`` on ``device`` when it is None."""
    if buf is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (buf.shape == shape and buf.dtype == dtype and buf.device == device and buf.is_contiguous()):
        raise ValueError('%s must be a contiguous %s tensor %s on %s' % (what, dtype, list(shape), device))
    return buf


def _det_buffers(B, max_det, device, index=True):
    """Outputs of an NMS / merge launch: (det [B,max_det,28] fp32, count [B] int32, index [B,max_det] int32 or None)."""
    return (torch.empty(B, max_det, abi.LP_DET_COLS, dtype=torch.float32, device=device),
            torch.empty(B, dtype=torch.int32, device=device),
            torch.empty(B, max_det, dtype=torch.int32, device=device) if index else None)


def _check_det_count(det, count, what='det', min_batch=0):
    """det [B >= min_batch, max_det, 28] fp32 and count [B] int32 as ``nms_padded`` returns them: contiguous, on one GPU."""
    if not (det.is_cuda and det.dtype == torch.float32 and det.dim() == 3 and det.shape[2] == abi.LP_DET_COLS
            and det.is_contiguous() and det.shape[0] >= min_batch):
        raise ValueError('%s must be a contiguous CUDA fp32 [B >= %d, max_det, 28] tensor' % (what, min_batch))
    if not (count.is_cuda and count.dtype == torch.int32 and count.is_contiguous() and count.numel() == det.shape[0]
            and count.device == det.device):
        raise ValueError('the count of %s must be a contiguous CUDA int32 [B] tensor on its device' % what)


def _check_ended(ended_i, ended_f, ended_count, device, what, also=()):
    """The ended records of a ``PlateTracker.update``: ended_i int32 / ended_f fp32 [S,max_ended,12] and ended_count int32 [S],
    contiguous on ``device`` like the tensors of ``also``; ``what`` is the sentence of the ValueError that names the device."""
    if ended_i.dim() != 3 or ended_i.shape[2] != 12 or ended_i.dtype != torch.int32 or ended_f.shape != ended_i.shape \
            or ended_f.dtype != torch.float32 or ended_count.dtype != torch.int32 or ended_count.shape != ended_i.shape[:1]:
        raise ValueError('ended_i int32 / ended_f fp32 must be [S,max_ended,12] and ended_count int32 [S]')
    for t in (ended_i, ended_f, ended_count) + tuple(also):
        if t.device != device or not t.is_contiguous():
            raise ValueError('%s %s' % (what, device))


def _unpad(det, counts, n=None):
    """The reference-shaped list of a padded result: det[b, :counts[b]] of the first ``n`` images (default: all), ``counts``
    being the host copy of the count tensor -- reading it is the caller's one host sync."""
    return [det[b, :counts[b]] for b in range(len(counts) if n is None else n)]


def _frames_device(frames):
    """The one device of a non-empty list of contiguous uint8 CUDA [h,w,3] frames (ValueError otherwise)."""
    dev = frames[0].device
    for f in frames:
        if not (f.is_cuda and f.device == dev and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
            raise ValueError('frames must be contiguous uint8 CUDA tensors [h, w, 3] on one device')
    return dev


def _nv12_device(frames):
    """The one device of a non-empty list of ``Nv12Frame`` whose planes are CUDA tensors (ValueError otherwise)."""
    dev = frames[0].device
    for f in frames:
        if not (isinstance(f, Nv12Frame) and f.is_cuda and f.device == dev):
            raise ValueError('NV12 frames must be Nv12Frame objects with CUDA planes on one device')
    return dev


def _frames_on(frames, what='frames'):
    """(device, is_nv12) of a non-empty list of frames of ONE kind: contiguous uint8 CUDA [h,w,3] BGR tensors, or ``Nv12Frame``
    objects with CUDA planes (a mixed list is a ValueError)."""
    if is_nv12_list(frames, what):
        return _nv12_device(frames), True
    return _frames_device(frames), False


def _batch_on(frames, n, dtype, batch, what):
    """Argument checks of a batched preprocess of ``n`` images cut from ``frames``: (device, B), where ``batch`` (>= n, >= 1)
    sets B and the slots past n are padding."""
    if dtype not in _DT:
        raise TypeError('unsupported input dtype %s' % dtype)
    if not frames:
        raise ValueError('%s needs at least one frame' % what)
    dev, _ = _frames_on(frames, what)
    B = n if batch is None else int(batch)
    if B < n or B < 1:
        raise ValueError('batch %d < %d images (or < 1)' % (B, n))
    return dev, B


def _plane_descs(desc_type, frames, nv12):
    """The ``desc_type`` array (lp_redact_desc's fields) of a checked frame list of one kind: the Y and UV planes of ``Nv12Frame``s
    (format 1) or the one plane of contiguous BGR tensors (format 0)."""
    desc = (desc_type * len(frames))()
    for d, f in zip(desc, frames):
        if nv12:
            d.p0, d.p1, d.pitch0, d.pitch1, d.format = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, 1
        else:
            d.p0, d.p1, d.pitch0, d.format = f.data_ptr(), None, 3 * f.shape[1], 0
        d.h0, d.w0 = f.shape[0], f.shape[1]
    return desc


def _desc_run(desc, b0):
    """Pointer to element ``b0`` of a ctypes descriptor array: what a launch over the run of frames that starts there takes."""
    return ctypes.cast(ctypes.byref(desc, b0 * ctypes.sizeof(desc._type_)), ctypes.POINTER(desc._type_))


def _runs_by_key(keys):
    """[(b0, b1), ...] of the maximal runs of equal consecutive ``keys``: one launch per run of frames that share its parameters."""
    runs, b0 = [], 0
    for b1 in range(1, len(keys) + 1):
        if b1 == len(keys) or keys[b1] != keys[b0]:
            runs.append((b0, b1))
            b0 = b1
    return runs


def _runs_under_cap(sizes, cap):
    """[(b0, b1), ...] of consecutive runs whose ``sizes`` sum to at most ``cap``; a run has at least one item, so an item above
    the cap goes alone: one launch per run of frames whose workspaces fit together."""
    runs, b0, total = [], 0, 0
    for b1, size in enumerate(sizes):
        if b1 > b0 and total + size > cap:
            runs.append((b0, b1))
            b0, total = b1, 0
        total += size
    if sizes:
        runs.append((b0, len(sizes)))
    return runs
