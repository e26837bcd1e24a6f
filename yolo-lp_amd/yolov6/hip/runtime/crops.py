"""Perspective-rectified plate crops and their sharpness (lp_plate_crops_batch, lp_crop_sharpness)."""
import numpy as np
import torch

from yolov6.hip import abi

from ._base import _buffer, _check_det_count, _dptr, _frames_device, _stream_ptr, _unpad
from .frames import _bgr_frames, detect_frames_padded


def _crop_size(crop_hw):
    Hc, Wc = (int(v) for v in crop_hw)
    if not (1 <= Hc <= 1024 and 1 <= Wc <= 1024):
        raise ValueError('crop size %dx%d: need 1..1024 on each side' % (Hc, Wc))
    return Hc, Wc


def _plate_crops_launch(frames, det, count, slots, out, status, crop_hw):
    """lp_plate_crops_batch on frames with ``slots[b]`` = (max_crops, out_slot): out [n_slots,Hc,Wc,3], status [n_slots]."""
    _check_det_count(det, count, min_batch=len(frames))
    if det.device != out.device:
        raise ValueError('det must be on the frames\' device')
    desc = (abi.CropDesc * len(frames))()
    for d, f, (m, o) in zip(desc, frames, slots):
        d.img, d.h0, d.w0, d.max_crops, d.out_slot = f.data_ptr(), f.shape[0], f.shape[1], m, o
    with torch.cuda.device(det.device):
        abi.check(abi.load().lp_plate_crops_batch(desc, len(frames), _dptr(det), _dptr(count), det.shape[1], _dptr(out),
                                                  _dptr(status), status.numel(), crop_hw[0], crop_hw[1], _stream_ptr(det.device)),
                  'lp_plate_crops_batch')


def plate_crops(frames, det, count, crop_hw=(64, 192), max_crops=None, out=None, status=None):
    """Perspective-rectified plate crops (lp_plate_crops_batch, one launch per 64 frames) of the detections of B frames:
    frame b (contiguous uint8 CUDA [h,w,3] BGR) is cut along its rows r < min(count[b], max_det, max_crops) of det
    [B,max_det,28] (fp32, source-frame pixels, as ``rescale_round_batch`` leaves them; count int32 [B] on the device, read by
    the kernel: no host sync).  Returns (crops [B,max_crops,Hc,Wc,3] uint8 BGR, status [B,max_crops] int32): 1 = cut along
    the four corners, 2 = along the box (the corners are not a convex quad of area >= 1), 3 = neither is usable (zeros),
    0 = no such detection (the crop's bytes are left as they were).  ``max_crops`` defaults to 16 (each slot is Hc*Wc*3
    bytes); ``out`` / ``status``: persistent buffers of those shapes.  yolov6.utils.plate_crop.plate_crops_np is the same
    computation on the CPU, bit for bit.  A list of ``Nv12Frame`` is converted with ``nv12_to_bgr`` first."""
    if not frames:
        raise ValueError('plate_crops needs at least one frame')
    frames = _bgr_frames(frames)            # an NV12 list is converted once, on this stream
    dev = _frames_device(frames)
    Hc, Wc = _crop_size(crop_hw)
    n, m = len(frames), 16 if max_crops is None else int(max_crops)
    if m < 0:
        raise ValueError('max_crops must be >= 0')
    out = _buffer(out, (n, m, Hc, Wc, 3), torch.uint8, dev)
    status = _buffer(status, (n, m), torch.int32, dev, 'status')
    _plate_crops_launch(frames, det, count, [(m, b * m) for b in range(n)], out, status, (Hc, Wc))
    return out, status


def crop_sharpness(crops, status, out=None):
    """Laplacian energy of plate crops (lp_crop_sharpness, one workgroup per crop): crops [..., Hc, Wc, 3] uint8 + status [...]
    int32 as ``plate_crops`` returns them -> int64 [...] on the device holding the unsigned 64-bit sums (view the host copy as
    uint64); 0 for status 0 or 3 or a side shorter than 3.  ``out``: a persistent buffer of that shape.
    yolov6.utils.best_shot.crop_sharpness_np is the same computation on the CPU, bit for bit."""
    if not (crops.is_cuda and crops.dtype == torch.uint8 and crops.dim() >= 3 and crops.shape[-1] == 3 and crops.is_contiguous()):
        raise ValueError('crops must be a contiguous uint8 CUDA tensor [..., Hc, Wc, 3]')
    lead = crops.shape[:-3]
    Hc, Wc = _crop_size(crops.shape[-3:-1])
    if not (status.dtype == torch.int32 and status.shape == lead and status.device == crops.device and status.is_contiguous()):
        raise ValueError('status must be a contiguous int32 tensor %s on the crops\' device' % list(lead))
    out = _buffer(out, lead, torch.int64, crops.device, 'sharp')
    with torch.cuda.device(crops.device):
        abi.check(abi.load().lp_crop_sharpness(_dptr(crops), _dptr(status), status.numel(), Hc, Wc, _dptr(out), _stream_ptr(crops.device)),
                  'lp_crop_sharpness')
    return out


def _unpad_with_crops(frames, det, count, crop_hw):
    """(dets, crops, status) of the ``*_with_crops`` entry points from a padded result in frame pixels: the one host read of
    the counts, then the crops packed, frame b's n_b right behind frame b-1's (``crop_hw``: checked by ``_crop_size``)."""
    frames = _bgr_frames(frames)            # an NV12 list is converted once, on this stream, before the host read
    counts = count.cpu().tolist()
    ns = [max(0, min(int(c), det.shape[1])) for c in counts[:len(frames)]]
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(int).tolist()
    crops = torch.empty(offs[-1], *crop_hw, 3, dtype=torch.uint8, device=det.device)
    status = torch.empty(offs[-1], dtype=torch.int32, device=det.device)
    _plate_crops_launch(frames, det, count, list(zip(ns, offs)), crops, status, crop_hw)
    return (_unpad(det, counts, len(frames)), [crops[o:o + k] for o, k in zip(offs, ns)],
            [status[o:o + k] for o, k in zip(offs, ns)])


def detect_frames_with_crops(model, frames, img_size, conf_thres, iou_thres, max_det, crop_hw=(64, 192), auto=True, batch=None,
                             out=None):
    """``detect_frames`` plus the plate crop of every detection: (dets, crops, status).  ``dets`` is bit for bit what
    ``detect_frames`` returns; after its one host read of the counts the crops are packed, frame b's n_b crops right behind
    frame b-1's in one [sum n_b,Hc,Wc,3] uint8 tensor: ``crops[b]`` is an [n_b,Hc,Wc,3] view of it and ``status[b]`` an
    [n_b] int32 view (codes as in ``plate_crops``).  The crops are enqueued here, before the next ``FrameBatcher.put`` may
    reuse the frames' buffer."""
    crop_hw = _crop_size(crop_hw)
    det, count = detect_frames_padded(model, frames, img_size, conf_thres, iou_thres, max_det, auto, batch, out)
    return _unpad_with_crops(frames, det, count, crop_hw)
