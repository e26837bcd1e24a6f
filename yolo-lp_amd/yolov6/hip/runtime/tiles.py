"""Tiled detection of large frames (yolov6/core/tiles.py plans the tiles; lp_preprocess_tiles_batch / lp_merge_tiles)."""
import ctypes

import torch

from yolov6.core.frames import letterbox_placement
from yolov6.core.tiles import hw_pair, plan_frames, tiles_per_frame
from yolov6.hip import abi

from ._base import _batch_on, _buffer, _check_det_count, _det_buffers, _dptr, _frames_on, _stream_ptr, _unpad
from .crops import _crop_size, _unpad_with_crops
from .engine import detect_padded
from .frames import _letterbox_regions, rescale_round_batch


def preprocess_tiles(frames, plans, img_size, stride, dtype, batch=None, out=None):
    """Letterboxed regions of device frames (lp_preprocess_tiles_batch, one launch per 64 tiles): ``plans`` is a list of
    (frame index, y0, x0, th, tw); tile k is read in place from ``frames[frame]`` (contiguous uint8 CUDA [h,w,3] BGR) and
    letterboxed to exactly ``img_size`` (the reference arithmetic of a (th, tw) image, ``auto=False``) into slot k of
    x [B,3,H,W] of ``dtype``: bit for bit what ``preprocess_frames(auto=False)`` gives for a contiguous copy of the region.
    Returns (x, geoms) with ``geoms[k]`` = (rh, rw, top, left).  ``batch`` (>= len(plans)) sets B, the slots past the tiles
    are padding (114/255); ``out``: a persistent [B,3,H,W] buffer to write."""
    dev, B = _batch_on(frames, len(plans), dtype, batch, 'preprocess_tiles')
    H, W = hw_pair(img_size)
    out = _buffer(out, (B, 3, H, W), dtype, dev)
    geoms = [letterbox_placement((th, tw), [H, W], stride, auto=False)[:4] for _, _, _, th, tw in plans]
    return _letterbox_regions(frames, plans, geoms, B, H, W, dtype, out, dev), geoms


_METRICS = {'iou': 0, 'ios': 1}


def merge_tiles_buffers(F, max_det, device):
    """New (det [F,max_det,28], count [F], src [F,max_det], workspace) of a ``merge_tiles`` of ``F`` frames: what its ``out`` takes."""
    need = abi.load().lp_merge_tiles_workspace_bytes(int(F), int(max_det))
    return _det_buffers(int(F), int(max_det), device) + (torch.empty(need + 16, dtype=torch.uint8, device=device),)


def merge_tiles(det_t, count_t, tiles, frame_shapes, thres, max_det, metric='iou', border=1, out=None):
    """Per-frame merge of per-tile detections on the device (lp_merge_tiles; no host sync): det_t [T',max_det_t,28] fp32 and
    count_t [T'] int32 hold the detections of tiles 0..len(tiles)-1 (T' >= len(tiles)) in tile-local source pixels, rounded;
    ``tiles[t]`` = (frame, y0, x0, th, tw) with a frame's tiles contiguous and frames ascending; ``frame_shapes[f]`` =
    (h, w[, c]).  Returns (det [F,max_det,28], count [F] int32, src [F,max_det] int32) in frame pixels -- the layout
    ``plate_crops`` takes.  Highest-scoring view wins; rows of one tile never suppress each other.
    ``yolov6.utils.tiles.merge_tiles_np`` is the same computation on the CPU, bit for bit, and states the rules.
    ``out``: persistent (det, count, src, workspace) of an earlier call of the same F and max_det to write instead of new tensors
    (``merge_tiles_buffers``), for callers that must not allocate."""
    _check_det_count(det_t, count_t, 'det_t', min_batch=len(tiles))
    if metric not in _METRICS:
        raise ValueError('metric must be one of %s' % sorted(_METRICS))
    dev, F, max_det = det_t.device, len(frame_shapes), int(max_det)
    if max_det < 1:
        raise ValueError('max_det must be >= 1')
    ref = (abi.TileRef * max(len(tiles), 1))()
    for r, (f, y0, x0, th, tw) in zip(ref, tiles):
        r.frame, r.y0, r.x0, r.th, r.tw = f, y0, x0, th, tw
    hw = (ctypes.c_int * max(2 * F, 1))(*[int(v) for s in frame_shapes for v in s[:2]])
    lib = abi.load()
    with torch.cuda.device(dev):
        need = lib.lp_merge_tiles_workspace_bytes(F, max_det)
        if out is None:
            det, count, src, ws = merge_tiles_buffers(F, max_det, dev)
        else:
            det, count, src, ws = out
            _check_det_count(det, count, 'out', min_batch=F)
            if det.shape != (F, max_det, abi.LP_DET_COLS) or det.device != dev or src.shape != (F, max_det) or ws.numel() < need + 16:
                raise ValueError('out must be the merge_tiles_buffers of %d frames and max_det %d on %s' % (F, max_det, dev))
        abi.check(lib.lp_merge_tiles(_dptr(det_t), _dptr(count_t), ref, len(tiles), det_t.shape[1], hw, F, float(thres),
                                     _METRICS[metric], int(border), max_det, _dptr(det), _dptr(count), _dptr(src),
                                     (ws.data_ptr() + 15) // 16 * 16, need, _stream_ptr(dev)), 'lp_merge_tiles')
    return det, count, src


_tile_inputs = {}      # (device, stream, dtype, B, H, W) -> persistent network input of the tile batches (graphs are keyed on the input pointer)


def plan_tiled(frame_shapes, img_size, max_det, tile_hw=None, overlap=0.2, overview=True, tile_max_det=None):
    """(tiles, tile_max_det) of ``detect_tiled`` for frames of ``frame_shapes``: the flat tile table (frame, y0, x0, th, tw)
    and the detections kept per tile, min(max_det, 16384 // most tiles of any frame) by default."""
    tiles = plan_frames(frame_shapes, hw_pair(img_size) if tile_hw is None else tile_hw, overlap, overview)
    most = max(tiles_per_frame(tiles, len(frame_shapes)))
    if most > abi.LP_MERGE_MAX_TILES:
        raise ValueError('%d tiles for one frame (at most %d): use larger tiles or a smaller overlap' % (most, abi.LP_MERGE_MAX_TILES))
    tmd = min(int(max_det), abi.LP_MERGE_MAX_CANDIDATES // most) if tile_max_det is None else int(tile_max_det)
    if tmd < 1:
        raise ValueError('tile_max_det must be >= 1')
    return tiles, tmd


def detect_tiles_padded(model, frames, tiles, img_size, conf_thres, iou_thres, tile_max_det, batch=32):
    """The per-tile half of ``detect_tiled``: the tiles (frame, y0, x0, th, tw) of ``frames`` in chunks of ``batch`` (the tail
    padded, so the engine is bound once) through ``preprocess_tiles`` -> ``detect_padded``, then one ``rescale_round_batch``
    over all tiles with each tile's (th, tw) as its source image.  Returns (det_t [T',tile_max_det,28], count_t [T']) on the
    device, T' = len(tiles) rounded up to a multiple of ``batch``; no host sync."""
    dev, _ = _frames_on(frames, 'detect_tiled')
    dtype = next(model.parameters()).dtype
    H, W = hw_pair(img_size)
    B = int(batch)
    if B < 1:
        raise ValueError('batch must be >= 1')
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, dtype, B, H, W)
    x = _tile_inputs.get(key)
    if x is None:
        x = _tile_inputs[key] = torch.empty(B, 3, H, W, dtype=dtype, device=dev)
    stride = int(model.stride.max())
    dets, counts = [], []
    for c0 in range(0, len(tiles), B):
        preprocess_tiles(frames, tiles[c0:c0 + B], [H, W], stride, dtype, batch=B, out=x)
        det, count, _ = detect_padded(model, x, conf_thres, iou_thres, tile_max_det)
        dets.append(det)
        counts.append(count)
    det_t = dets[0] if len(dets) == 1 else torch.cat(dets)
    count_t = counts[0] if len(counts) == 1 else torch.cat(counts)
    rescale_round_batch(det_t, count_t, (H, W), [(t[3], t[4]) for t in tiles])
    return det_t, count_t


def detect_tiled_padded(model, frames, img_size, conf_thres, iou_thres, max_det, tile_hw=None, overlap=0.2, overview=True,
                        metric='iou', border=1, batch=32, tile_max_det=None):
    """The device work of ``detect_tiled`` without its host read: (det [F,max_det,28], count [F] int32) on the device, in
    frame pixels."""
    if not frames:
        raise ValueError('detect_tiled needs at least one frame')
    shapes = [tuple(f.shape[:2]) for f in frames]
    tiles, tmd = plan_tiled(shapes, img_size, max_det, tile_hw, overlap, overview, tile_max_det)
    det_t, count_t = detect_tiles_padded(model, frames, tiles, img_size, conf_thres, iou_thres, tmd, batch)
    det, count, _ = merge_tiles(det_t, count_t, tiles, shapes, iou_thres, max_det, metric, border)
    return det, count


def detect_tiled(model, frames, img_size, conf_thres, iou_thres, max_det, tile_hw=None, overlap=0.2, overview=True, metric='iou',
                 border=1, batch=32, tile_max_det=None):
    """Detections of large frames (contiguous uint8 CUDA [h,w,3] BGR, any sizes) by tiles: every frame is sliced into
    overlapping ``tile_hw`` tiles (default: the network input size, so a tile maps 1:1 to network pixels) plus, with
    ``overview``, the whole frame (``yolov6.core.tiles.plan_tiles``); the tiles of all frames run through the engine ``batch``
    at a time; the per-tile detections are rescaled to tile pixels, shifted and merged per frame on the device
    (``merge_tiles``: threshold ``iou_thres``, ``metric`` 'iou' or 'ios', cut-plate ``border``), then ONE host read of the
    per-frame counts.  Returns a list of [n_f, 28] tensors in frame pixels.  ``tile_max_det``: detections kept per tile
    (default min(max_det, 16384 // most tiles of any frame)).  With ``tile_hw`` >= the frame this is
    ``detect_frames(auto=False)``, bit for bit.  ``frames`` may be a list of ``Nv12Frame`` instead: the tiles are cut from the planes
    (lp_preprocess_nv12_batch) and the result equals that of the converted frames."""
    det, count = detect_tiled_padded(model, frames, img_size, conf_thres, iou_thres, max_det, tile_hw, overlap, overview, metric,
                                     border, batch, tile_max_det)
    return _unpad(det, count.cpu().tolist())


def detect_tiled_with_crops(model, frames, img_size, conf_thres, iou_thres, max_det, crop_hw=(64, 192), tile_hw=None, overlap=0.2,
                            overview=True, metric='iou', border=1, batch=32, tile_max_det=None):
    """``detect_tiled`` plus the plate crop of every merged detection, cut from the full-resolution frame: (dets, crops, status)
    packed as ``detect_frames_with_crops`` packs them (``plate_crops`` on the merged det / count, which have its layout)."""
    crop_hw = _crop_size(crop_hw)
    det, count = detect_tiled_padded(model, frames, img_size, conf_thres, iou_thres, max_det, tile_hw, overlap, overview, metric,
                                     border, batch, tile_max_det)
    return _unpad_with_crops(frames, det, count, crop_hw)
