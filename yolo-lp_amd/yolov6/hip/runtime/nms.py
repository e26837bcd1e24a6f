"""NMS on the device (lp_nms on the prediction tensor, lp_nms_candidates on the candidate lists of the detections-only forward)
and the counters of the LP accuracy metric (lp_eval_counts)."""
import torch

from yolov6.hip import abi

from ._base import _aligned, _check_det_count, _det_buffers, _dptr, _stream_ptr, _stream_workspace, _unpad

_nms_ws = {}


def _nms_workspace(device, need):
    """The NMS workspace of ``device``'s current stream, grown to ``need`` bytes (+ 256 for ``_aligned``)."""
    # one workspace per (device, stream): lp_nms memsets and fills it on the current stream, so two streams must never
    # share one; a regrown buffer is released through the caching allocator, which orders its reuse on this stream
    return _stream_workspace(_nms_ws, device, need)


def nms_candidates(handle, iou_thres, max_det, want_keep=False):
    """Second half of the NMS (lp_nms_candidates: sort, > 30000 cut, greedy suppression, max_det) on the current stream for the
    candidate lists ``Engine.forward_det`` left in its workspace: (det[B,max_det,28], count[B] int32, keep or None)."""
    ws, B, N = handle
    if not 0.0 <= iou_thres <= 1.0:
        raise ValueError('iou_thres must be in [0, 1]')
    lib = abi.load()
    dev = ws.device
    with torch.cuda.device(dev):
        need = lib.lp_nms_workspace_bytes(B, N)
        det, count, keep = _det_buffers(B, max_det, dev, want_keep)
        abi.check(lib.lp_nms_candidates(B, N, float(iou_thres), int(max_det), _dptr(det), _dptr(count), _dptr(keep), _aligned(ws),
                                        need, _stream_ptr(dev)), 'lp_nms_candidates')
    return det, count, keep


def nms_padded(prediction, conf_thres, iou_thres, max_det, want_keep=False):
    """Batch NMS through lp_nms without a host sync: (det[B,max_det,28], count[B] int32, keep or None)."""
    if not (prediction.is_cuda and prediction.dtype == torch.float32 and prediction.is_contiguous()):
        raise ValueError('prediction must be a contiguous fp32 CUDA tensor')
    B, N, C = prediction.shape
    if C != abi.LP_PRED_COLS:
        raise ValueError('prediction must have %d columns, got %d' % (abi.LP_PRED_COLS, C))
    lib = abi.load()
    dev = prediction.device
    with torch.cuda.device(dev):
        need = lib.lp_nms_workspace_bytes(B, N)
        ws = _nms_workspace(dev, need)
        det, count, keep = _det_buffers(B, max_det, dev, want_keep)
        abi.check(lib.lp_nms(_dptr(prediction), B, N, float(conf_thres), float(iou_thres), int(max_det), _dptr(det), _dptr(count),
                             _dptr(keep), _aligned(ws), need, _stream_ptr(dev)), 'lp_nms')
    return det, count, keep


def non_max_suppression(prediction, conf_thres, iou_thres, max_det):
    """Reference-shaped result: list (len B) of [n_i, 28] tensors; one host sync for the whole batch."""
    B, N = prediction.shape[0], prediction.shape[1]
    if B == 0 or N == 0:
        return [torch.zeros((0, 28), device=prediction.device)] * B
    src = prediction
    work = prediction
    if work.dtype != torch.float32 or not work.is_contiguous():
        work = work.float().contiguous()
    det, count, _ = nms_padded(work, conf_thres, iou_thres, max_det)
    if work is not src:
        src.copy_(work)          # keep the reference's in-place obj*cls side effect on the caller's tensor
    return _unpad(det, count.cpu().tolist())


def eval_counts(det, det_count, tgt, tgt_count, counts=None):
    """Counters of the LP accuracy metric for one batch (``lp_eval_counts``): det [B,max_det,28] fp32 + det_count [B]
    int32 as ``nms_padded`` returns them, tgt [B,max_t,20] fp32 + tgt_count [B] int32; ``counts`` (int64 [43], CUDA) is
    accumulated into and returned (allocated zeroed when None)."""
    dev = det.device
    _check_det_count(det, det_count)
    if not (tgt.dtype == torch.float32 and tgt.dim() == 3 and tgt.shape[2] == 20 and tgt.is_contiguous() and tgt.device == dev
            and tgt_count.dtype == torch.int32 and tgt_count.is_contiguous() and tgt_count.device == dev
            and det.shape[0] == tgt.shape[0] == tgt_count.numel()):
        raise ValueError('eval_counts: expected contiguous CUDA tgt [B,T,20] fp32 and int32 tgt_count [B] on det\'s device')
    if counts is None:
        counts = torch.zeros(abi.LP_EVAL_NCOUNTS, dtype=torch.int64, device=dev)
    elif not (counts.dtype == torch.int64 and counts.numel() == abi.LP_EVAL_NCOUNTS and counts.device == dev and counts.is_contiguous()):
        raise ValueError('eval_counts: counts must be a contiguous CUDA int64 [%d] tensor' % abi.LP_EVAL_NCOUNTS)
    with torch.cuda.device(dev):
        abi.check(abi.load().lp_eval_counts(_dptr(det), _dptr(det_count), det.shape[1], _dptr(tgt), _dptr(tgt_count), tgt.shape[1],
                                            det.shape[0], _dptr(counts), _stream_ptr(dev)), 'lp_eval_counts')
    return counts
