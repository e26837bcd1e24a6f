"""Raw frames in, detections out: NV12 conversion, the letterbox of frames and regions, the rescale back to source pixels and
``detect_frames`` (lp_nv12_to_bgr_batch, lp_preprocess_*_batch, lp_rescale_round*)."""
import torch

from yolov6.core.frames import letterbox_placement
from yolov6.hip import abi
from yolov6.utils.nv12 import Nv12Frame, is_nv12_list

from ._base import _DT, _batch_on, _buffer, _check_det_count, _dptr, _nv12_device, _stream_ptr, _unpad
from .engine import detect_padded


def nv12_to_bgr(frames, out=None):
    """BGR device frames of a list of ``Nv12Frame`` with CUDA planes on one device (lp_nv12_to_bgr_batch, one launch per 64
    frames, on the current stream): a list of contiguous uint8 [h,w,3] tensors, bit for bit ``nv12_to_bgr_np`` of each frame.
    For the callers that need the frame itself -- plate crops, the best-shot gallery, saving images; detection reads NV12
    directly.  ``out``: a list of persistent [h,w,3] uint8 buffers to write (any alignment); by default the frames are views
    of one new buffer, at 256-byte aligned bases."""
    if not frames:
        return []
    dev = _nv12_device(frames)
    if out is None:
        offs, n = [], 0
        for f in frames:
            offs.append(n)
            n += (f.h * f.w * 3 + 255) // 256 * 256
        buf = torch.empty(n, dtype=torch.uint8, device=dev)
        out = [buf[o:o + f.h * f.w * 3].view(f.h, f.w, 3) for f, o in zip(frames, offs)]
    else:
        out = list(out)
        if len(out) != len(frames):
            raise ValueError('%d output buffers for %d frames' % (len(out), len(frames)))
        out = [_buffer(o, (f.h, f.w, 3), torch.uint8, dev, 'out[%d]' % k) for k, (o, f) in enumerate(zip(out, frames))]
    desc = (abi.Nv12BgrDesc * len(frames))()
    for d, f, o in zip(desc, frames, out):
        d.y, d.uv, d.pitch_y, d.pitch_uv, d.h0, d.w0 = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, f.h, f.w
        d.matrix, d.out = f.matrix_id, o.data_ptr()
    with torch.cuda.device(dev):
        abi.check(abi.load().lp_nv12_to_bgr_batch(desc, len(frames), _stream_ptr(dev)), 'lp_nv12_to_bgr_batch')
    return out


def _bgr_frames(frames):
    """``frames`` as BGR device frames: an NV12 list converted once (``nv12_to_bgr``), a BGR list as it is; None entries stay."""
    live = [f for f in frames if f is not None]
    if not live or not is_nv12_list(live):
        return frames
    it = iter(nv12_to_bgr(live))
    return [None if f is None else next(it) for f in frames]


def _letterbox_regions(frames, plans, geoms, B, H, W, dtype, out, dev):
    """One letterbox call: region ``plans[k]`` = (frame index, y0, x0, th, tw) of ``frames`` with the letterbox geometry ``geoms[k]``
    = (rh, rw, top, left) into slot k of ``out`` [B,3,H,W].  BGR tensors go through lp_preprocess_tiles_batch; ``Nv12Frame``s through
    lp_preprocess_nv12_batch (the same kernel reading the planes: no BGR frame is created)."""
    for k, *_ in plans:
        if not 0 <= k < len(frames):
            raise ValueError('tile of frame %d: %d frames' % (k, len(frames)))
    nv12 = isinstance(frames[0], Nv12Frame)
    desc = ((abi.Nv12Desc if nv12 else abi.TileDesc) * max(len(plans), 1))()
    for d, (k, y0, x0, th, tw), (rh, rw, top, left) in zip(desc, plans, geoms):
        f = frames[k]
        if nv12:
            d.y, d.uv, d.pitch_y, d.pitch_uv, d.matrix = f.y.data_ptr(), f.uv.data_ptr(), f.pitch_y, f.pitch_uv, f.matrix_id
        else:
            d.img = f.data_ptr()
        d.h0, d.w0, d.y0, d.x0, d.th, d.tw, d.rh, d.rw, d.top, d.left = f.shape[0], f.shape[1], y0, x0, th, tw, rh, rw, top, left
    name = 'lp_preprocess_nv12_batch' if nv12 else 'lp_preprocess_tiles_batch'
    with torch.cuda.device(dev):
        abi.check(getattr(abi.load(), name)(desc, len(plans), B, _dptr(out), _DT[dtype], H, W, _stream_ptr(dev)), name)
    return out


def preprocess_letterbox(frame_bgr_u8, img_size, stride, dtype, auto=True):
    """GPU form of Inferer.precess_image: device uint8 [h,w,3] BGR frame -> [3,H,W] RGB /255 tensor of ``dtype``.
    Geometry (ratio, resized size, padding) is the reference's letterbox arithmetic, done on the host; ``auto=False``
    pads to exactly ``img_size`` instead of the next stride multiple."""
    if not (frame_bgr_u8.is_cuda and frame_bgr_u8.dtype == torch.uint8 and frame_bgr_u8.dim() == 3 and
            frame_bgr_u8.shape[2] == 3 and frame_bgr_u8.is_contiguous()):
        raise ValueError('frame must be a contiguous uint8 CUDA tensor [h, w, 3]')
    h0, w0 = frame_bgr_u8.shape[:2]
    rh, rw, top, left, H, W = letterbox_placement((h0, w0), img_size, stride, auto)
    out = torch.empty(3, H, W, dtype=dtype, device=frame_bgr_u8.device)
    with torch.cuda.device(out.device):
        abi.check(abi.load().lp_preprocess_letterbox(_dptr(frame_bgr_u8), h0, w0, _dptr(out), _DT[dtype], H, W, rh, rw, top, left,
                                                     _stream_ptr(out.device)), 'lp_preprocess_letterbox')
    return out


def preprocess_frames(frames, img_size, stride, dtype, auto=True, batch=None, out=None):
    """Batched ``preprocess_letterbox`` (each frame as the region (0, 0, h, w) of lp_preprocess_tiles_batch, which is
    lp_preprocess_letterbox_batch on whole frames; one launch per 64 frames): a list of contiguous
    uint8 CUDA [h,w,3] BGR frames of any sizes -> (x[B,3,H,W] of ``dtype``, geoms).  ``geoms[i]`` is frame i's
    (rh, rw, top, left) from the host letterbox arithmetic.  With ``auto=True`` every frame must letterbox to the same
    (H, W); ``auto=False`` letterboxes each to exactly ``img_size``.  ``batch`` (>= len(frames)) sets B: slots past the
    frames are padding (114/255).  ``out``: a persistent [B,3,H,W] input buffer to write (graphs are keyed on the
    input pointer).  A list of ``Nv12Frame`` (CUDA planes) is taken instead of BGR tensors: the conversion is fused into the
    letterbox (lp_preprocess_nv12_batch) and x equals, bit for bit, that of the frames ``nv12_to_bgr`` gives."""
    dev, B = _batch_on(frames, len(frames), dtype, batch, 'preprocess_frames')
    places = [letterbox_placement(f.shape, img_size, stride, auto) for f in frames]
    geoms, hws = [p[:4] for p in places], set(p[4:] for p in places)
    if len(hws) != 1:
        raise ValueError('frames letterbox to different shapes %s (source shapes %s): batch them separately or use auto=False'
                         % (sorted(hws), [tuple(f.shape[:2]) for f in frames]))
    H, W = hws.pop()
    out = _buffer(out, (B, 3, H, W), dtype, dev)
    plans = [(k, 0, 0) + tuple(f.shape[:2]) for k, f in enumerate(frames)]      # a whole frame: the region (0, 0, h, w)
    return _letterbox_regions(frames, plans, geoms, B, H, W, dtype, out, dev), geoms


def _rescale_terms(ori_shape, target_shape):
    """Inferer.rescale's (ratio, padx, pady) from the network input (h, w) back to a source image of (h, w[, c])."""
    ratio = min(ori_shape[0] / target_shape[0], ori_shape[1] / target_shape[1])
    return ratio, (ori_shape[1] - target_shape[1] * ratio) / 2, (ori_shape[0] - target_shape[0] * ratio) / 2


def rescale_round(ori_shape, det, target_shape):
    """GPU form of ``Inferer.rescale(ori_shape, det[:, :12], target_shape).round()``, in place on det [n, 28]."""
    if not (det.is_cuda and det.dtype == torch.float32 and det.dim() == 2 and det.shape[1] == abi.LP_DET_COLS and
            det.stride(1) == 1 and det.stride(0) == abi.LP_DET_COLS):
        raise ValueError('det must be a CUDA fp32 [n, 28] tensor with contiguous rows')
    ratio, padx, pady = _rescale_terms(ori_shape, target_shape)
    with torch.cuda.device(det.device):
        abi.check(abi.load().lp_rescale_round(_dptr(det), det.shape[0], float(ratio), float(padx), float(pady),
                                              int(target_shape[1]), int(target_shape[0]), _stream_ptr(det.device)),
                  'lp_rescale_round')
    return det


def rescale_round_batch(det, count, net_hw, src_shapes):
    """Batched ``rescale_round`` (lp_rescale_round_batch), in place on det [B,max_det,28]: rows r < count[b] of image
    b < len(src_shapes) are mapped back to source image b of shape (h, w[, c]) from the network input size ``net_hw``
    (Inferer.rescale's ratio and padding) and rounded.  ``count`` (int32 [B], CUDA) is read on the device: no host sync."""
    _check_det_count(det, count)
    n = len(src_shapes)
    if n > det.shape[0]:
        raise ValueError('%d source shapes for a batch of %d' % (n, det.shape[0]))
    desc = (abi.RescaleDesc * max(n, 1))()
    for d, s in zip(desc, src_shapes):
        d.ratio, d.padx, d.pady = _rescale_terms(net_hw, s)
        d.img_w, d.img_h = int(s[1]), int(s[0])
    with torch.cuda.device(det.device):
        abi.check(abi.load().lp_rescale_round_batch(_dptr(det), _dptr(count), n, det.shape[1], desc, _stream_ptr(det.device)),
                  'lp_rescale_round_batch')
    return det


def detect_frames_padded(model, frames, img_size, conf_thres, iou_thres, max_det, auto=True, batch=None, out=None):
    """The device work of ``detect_frames`` without its host read: (det [B,max_det,28], count [B] int32) on the device, rows
    r < count[b] of frame b < len(frames) in source-image pixels, rounded."""
    dtype = next(model.parameters()).dtype
    x, _ = preprocess_frames(frames, img_size, int(model.stride.max()), dtype, auto=auto, batch=batch, out=out)   # DetectBackend's stride
    det, count, _ = detect_padded(model, x, conf_thres, iou_thres, max_det)
    rescale_round_batch(det, count, x.shape[2:], [tuple(f.shape[:2]) for f in frames])
    return det, count


def detect_frames(model, frames, img_size, conf_thres, iou_thres, max_det, auto=True, batch=None, out=None):
    """Detections of a batch of raw frames (contiguous uint8 CUDA [h,w,3] BGR, any sizes that letterbox to one shape, or any
    sizes with ``auto=False``): ``preprocess_frames`` -> ``detect_padded`` -> ``rescale_round_batch``, then one host read of
    the counts.  Returns a list of [n_i, 28] tensors in source-image pixels, rounded: per frame what Inferer.infer returns,
    bit for bit.  The input dtype is the model's parameter dtype (Inferer's fp16 / fp32 input); ``batch`` / ``out`` as in
    ``preprocess_frames`` (padding slots let a short tail reuse a bound batch size).  ``frames`` may be a list of ``Nv12Frame``
    instead (the conversion is fused into the letterbox; no BGR frame is created): the result is, bit for bit, that of the frames
    ``nv12_to_bgr`` gives."""
    det, count = detect_frames_padded(model, frames, img_size, conf_thres, iou_thres, max_det, auto, batch, out)
    return _unpad(det, count.cpu().tolist(), len(frames))
