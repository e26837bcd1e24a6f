"""Plate redaction in place on the device: mosaic, fill and Gaussian blur (lp_redact_plates_batch, lp_redact_gauss_batch;
yolov6/utils/redact.py is the specification)."""
import ctypes

import torch

from yolov6.hip import abi

from ._base import (_aligned, _buffer, _check_det_count, _desc_run, _dptr, _frames_on, _plane_descs, _runs_by_key, _runs_under_cap,
                    _stream_ptr, _stream_workspace)

#: redact_plates(mode='gauss'): the tables of one lp_redact_gauss_batch call stay under this many bytes (a 4K frame takes 33 MB)
GAUSS_WS_CAP = 256 << 20
_redact_ws = {}


def _redact_workspace(device, need):
    """The cell table of ``redact_plates`` on ``device``'s current stream, grown to ``need`` bytes (+ 256 for ``_aligned``); one per
    (device, stream), as ``_nms_workspace``.  It needs no zeroing: a call reads only entries it has written itself."""
    return _stream_workspace(_redact_ws, device, need)


def redact_plates(frames, det, count, mode='mosaic', cell=16, margin=0.1, fill=(0, 0, 0), status=None, sigma=None):
    """Make the plates of B device frames unreadable IN PLACE (lp_redact_plates_batch, two launches per 64 frames on the current
    stream, no host read): ``frames`` is a list of contiguous uint8 CUDA [h,w,3] BGR tensors or of ``Nv12Frame`` with CUDA planes
    (one kind; NV12 is redacted in its own planes, no BGR copy exists), ``det`` [>= B,max_det,28] + ``count`` int32 on the device
    as ``detect_frames_padded``, ``detect_tiled_padded`` or ``PlateTracker.update`` (det_out) return them.  EVERY row
    r < min(max(count[b], 0), max_det) of frame b is redacted -- there is no cap -- along its corners, or its box when the
    corners are no convex quad of area >= 1, scaled by ``1 + margin`` about the centre.  ``mode`` 'mosaic': a pixel takes the mean of
    its ``cell`` x ``cell`` cell (even, 2..64; the grid is anchored to the frame, the means are of the frame before the call, so
    overlapping plates and the order of the rows do not matter); 'fill': ``fill`` = (B, G, R), converted with the frame's matrix
    for NV12; 'gauss': a pixel takes the frame as it was before the call under the integer Gaussian of ``sigma`` (0.5..16, None:
    8.0; lp_redact_gauss_batch, whose table takes 4 bytes per frame pixel: the frames go in runs whose tables stay under
    ``GAUSS_WS_CAP``), so the order of the rows and overlaps do not matter either, but a second call blurs again.
    Writes into the caller's tensors and returns status [B,max_det] int32: 1 = corners, 2 = box, 3 = neither usable
    (nothing written), 0 = no such row.  yolov6.utils.redact.redact_plates_np is the same computation on the CPU, bit for bit.

    REDACTION GOES LAST: ``plate_crops``, ``PlateTracker.update_with_shots`` and the best-shot gallery must read the frames
    BEFORE this call on the same stream, or they cut mosaics."""
    from yolov6.utils.redact import check_params, check_sigma, fill_bytes
    if not frames:
        raise ValueError('redact_plates needs at least one frame')
    dev, nv12 = _frames_on(frames, 'redact_plates')
    _check_det_count(det, count, min_batch=len(frames))
    if det.device != dev or det.shape[1] < 1:
        raise ValueError('det must be on the frames\' device with max_det >= 1')
    m, cell, margin = check_params(mode, cell, margin)
    n, max_det = len(frames), det.shape[1]
    status = _buffer(status, (n, max_det), torch.int32, dev, 'status')
    desc = _plane_descs(abi.RedactDesc, frames, nv12)
    if m == 2:
        with torch.cuda.device(dev):
            _redact_gauss(desc, [4 * f.shape[0] * f.shape[1] + 16 for f in frames], det, count, status, margin, check_sigma(sigma), dev)
        return status
    # one call per run of frames that share the fill's bytes: a BGR list or a mosaic is one run, an NV12 fill one per matrix
    fills = [fill_bytes(fill, f.matrix if nv12 and m == 1 else None) for f in frames]
    lib = abi.load()
    with torch.cuda.device(dev):
        for b0, b1 in _runs_by_key(fills):
            params = abi.RedactParams(m, cell, margin, (ctypes.c_ubyte * 3)(*fills[b0]))
            run = _desc_run(desc, b0)
            need = lib.lp_redact_workspace_bytes(run, b1 - b0, ctypes.byref(params))
            ws = _redact_workspace(dev, need) if m == 0 else None
            abi.check(lib.lp_redact_plates_batch(run, b1 - b0, _dptr(det[b0:b1]), _dptr(count[b0:b1]), max_det, ctypes.byref(params),
                                                 _dptr(status[b0:b1]), None if ws is None else _aligned(ws), need, _stream_ptr(dev)),
                      'lp_redact_plates_batch')
    return status


def _gauss_params(margin, sigma):
    """lp_redact_gauss_params of a public sigma: the taps of sigma for BGR and Y, of sigma / 2 for U and V."""
    from yolov6.utils.redact import gauss_taps
    t, tc = gauss_taps(sigma), gauss_taps(sigma / 2)
    p = abi.RedactGaussParams(margin, len(t) - 1, len(tc) - 1)
    p.taps[:len(t)] = [int(v) for v in t]
    p.taps_c[:len(tc)] = [int(v) for v in tc]
    return p


def _redact_gauss(desc, table_bytes, det, count, status, margin, sigma, dev):
    """lp_redact_gauss_batch over consecutive runs of the frames of ``desc`` whose tables (``table_bytes`` bounds each frame's) stay
    under ``GAUSS_WS_CAP`` together, at least one frame per run: frames are independent, so the split does not show."""
    lib, params, max_det = abi.load(), _gauss_params(margin, sigma), det.shape[1]
    for b0, b1 in _runs_under_cap(table_bytes, GAUSS_WS_CAP):
        run = _desc_run(desc, b0)
        need = lib.lp_redact_gauss_workspace_bytes(run, b1 - b0, ctypes.byref(params))
        ws = _redact_workspace(dev, need)
        abi.check(lib.lp_redact_gauss_batch(run, b1 - b0, _dptr(det[b0:b1]), _dptr(count[b0:b1]), max_det, ctypes.byref(params),
                                            _dptr(status[b0:b1]), _aligned(ws), need, _stream_ptr(dev)), 'lp_redact_gauss_batch')
