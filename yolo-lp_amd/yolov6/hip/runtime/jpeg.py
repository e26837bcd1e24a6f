"""Baseline JPEG files written on the device (yolov6/utils/jpeg.py is the specification; lp_jpeg_encode_batch)."""
import ctypes

import numpy as np
import torch

from yolov6.hip import abi
from yolov6.utils.nv12 import Nv12Frame

from ._base import _aligned, _desc_run, _dptr, _runs_under_cap, _stream_ptr, _stream_workspace
from .frames import nv12_to_bgr

#: encode_jpeg_padded: the workspace of one lp_jpeg_encode_batch call stays under this many bytes (a 4K frame takes 25 MB)
JPEG_WS_CAP = 256 << 20
#: 'retries': frames ``encode_jpeg`` encoded a second time because their file did not fit the first capacity
jpeg_stats = {'retries': 0}
_jpeg_ws = {}


def _jpeg_sources(frames):
    """The frames of one ``encode_jpeg`` call as (device, flat list of [h,w,3] tensors and 'bt601f' ``Nv12Frame``s): uint8 CUDA BGR
    tensors [h,w,3] of any sizes whose pixels are contiguous (a row pitch above 3 w is fine: views of a larger tensor), [n,h,w,3]
    tensors (n frames each), or ``Nv12Frame``s with CUDA planes; NV12 frames of a matrix other than 'bt601f' are converted to
    BGR frames here (``nv12_to_bgr``)."""
    if torch.is_tensor(frames):
        frames = [frames]
    flat = []
    for f in frames:
        if torch.is_tensor(f) and f.dim() == 4:
            flat.extend(f[k] for k in range(f.shape[0]))
        else:
            flat.append(f)
    if not flat:
        raise ValueError('encode_jpeg needs at least one frame')
    dev = flat[0].device
    other = [k for k, f in enumerate(flat) if isinstance(f, Nv12Frame) and f.matrix != 'bt601f']
    if other:
        for k, bgr in zip(other, nv12_to_bgr([flat[k] for k in other])):
            flat[k] = bgr
    for f in flat:
        if isinstance(f, Nv12Frame):
            if not (f.is_cuda and f.device == dev):
                raise ValueError('NV12 frames must be Nv12Frame objects with CUDA planes on one device')
            continue
        if not (torch.is_tensor(f) and f.is_cuda and f.device == dev and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3
                and f.shape[0] >= 1 and f.shape[1] >= 1 and f.stride(2) == 1 and f.stride(1) == 3 and f.stride(0) >= 3 * f.shape[1]):
            raise ValueError('frames must be uint8 CUDA BGR tensors [h, w, 3] (rows may be pitched) or [n, h, w, 3], on one device')
    for f in flat:
        if not (1 <= f.shape[0] <= 65535 and 1 <= f.shape[1] <= 65535):
            raise ValueError('JPEG sizes are 1..65535, got %d x %d' % (f.shape[0], f.shape[1]))
    return dev, flat


def encode_jpeg_padded(frames, quality=90, restart=16, cap=None):
    """Baseline JPEG files of device frames, left on the device (lp_jpeg_encode_batch, four launches per 32 frames on the current
    stream, no host read): (out uint8 [n, cap], nbytes int32 [n]); ``out[k, :nbytes[k]]`` is the complete file of frame k, byte
    for byte ``yolov6.utils.jpeg.encode_jpeg_np`` of it.  ``frames``: see ``encode_jpeg``.  ``cap``: bytes per file (None:
    ``h * w * 3 // 4 + 4096`` of the largest frame); a file that needs more leaves ``nbytes[k] = -needed`` and nothing written.
    The frames go in runs whose workspace (3 bytes per padded pixel) stays under ``JPEG_WS_CAP``."""
    from yolov6.utils.jpeg import check_params, jpeg_header
    quality, restart = check_params(quality, restart, device=True)
    dev, flat = _jpeg_sources(frames)
    n = len(flat)
    if cap is None:
        cap = max(f.shape[0] * f.shape[1] for f in flat) * 3 // 4 + 4096
    cap = int(cap)
    if not 1 <= cap < 1 << 31:
        raise ValueError('cap must be in 1..2^31-1, got %d' % cap)
    heads = np.stack([np.frombuffer(jpeg_header(f.shape[0], f.shape[1], quality, restart), np.uint8) for f in flat])
    desc = (abi.JpegDesc * n)()
    for d, f in zip(desc, flat):
        if isinstance(f, Nv12Frame):
            d.p0, d.p1, d.pitch0, d.pitch1, d.format, d.matrix = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, 1, f.matrix_id
        else:
            d.p0, d.p1, d.pitch0, d.pitch1, d.format, d.matrix = f.data_ptr(), None, f.stride(0), 0, 0, 0
        d.h0, d.w0 = f.shape[0], f.shape[1]
    lib, params = abi.load(), abi.JpegParams(quality, restart)
    with torch.cuda.device(dev):
        headers = torch.from_numpy(heads).to(dev)
        out = torch.empty((n, cap), dtype=torch.uint8, device=dev)
        nbytes = torch.empty(n, dtype=torch.int32, device=dev)
        ws_of = [(f.shape[0] + 15) // 16 * ((f.shape[1] + 15) // 16) * 776 + 16 for f in flat]     # an upper bound per frame
        for b0, b1 in _runs_under_cap(ws_of, JPEG_WS_CAP):
            run = _desc_run(desc, b0)
            need = lib.lp_jpeg_workspace_bytes(run, b1 - b0, restart)
            ws = _stream_workspace(_jpeg_ws, dev, need)
            abi.check(lib.lp_jpeg_encode_batch(run, b1 - b0, ctypes.byref(params), _dptr(headers[b0:b1]), heads.shape[1], _dptr(out[b0:b1]),
                                               cap, _dptr(nbytes[b0:b1]), _aligned(ws), need, _stream_ptr(dev)), 'lp_jpeg_encode_batch')
    return out, nbytes


def encode_jpeg(frames, quality=90, restart=16, cap=None):
    """Baseline JPEG files (a list of ``bytes``) of device frames: 4:2:0, the Annex K tables scaled by ``quality`` 1..100 as
    libjpeg scales them, restart intervals of ``restart`` MCUs (1..32).  ``frames``: a list of uint8 CUDA BGR tensors [h,w,3] of
    any sizes (rows may be pitched: views of a larger tensor), of [n,h,w,3] crop tensors, or of ``Nv12Frame``s with CUDA planes
    ('bt601f' planes feed the transform as they are; the other matrices are converted to a BGR frame first); a single tensor is
    a list of one.  Two host reads: ``nbytes``, then the used bytes.  ``cap`` as ``encode_jpeg_padded``; a frame whose file does
    not fit is encoded again at the capacity it reported, counted in ``jpeg_stats['retries']``."""
    dev, flat = _jpeg_sources(frames)
    out, nbytes = encode_jpeg_padded(flat, quality, restart, cap)
    nb = nbytes.cpu().tolist()
    files = [None] * len(flat)
    again = [k for k, v in enumerate(nb) if v < 0]
    if again:
        jpeg_stats['retries'] += len(again)
        for k, data in zip(again, encode_jpeg([flat[k] for k in again], quality, restart, max(-nb[k] for k in again))):
            files[k] = data
    most = max([v for v in nb if v > 0], default=0)
    if most:
        host = out[:, :most].cpu().numpy()
        for k, v in enumerate(nb):
            if v > 0:
                files[k] = host[k, :v].tobytes()
    return files
