"""Annotation overlay drawn on the device (yolov6/utils/overlay.py is the specification; lp_overlay_draw_batch)."""
import ctypes

import numpy as np
import torch

from yolov6.hip import abi

from ._base import (_aligned, _buffer, _check_det_count, _cuda_device, _desc_run, _dptr, _frames_on, _plane_descs, _runs_by_key,
                    _stream_ptr, _stream_workspace)

_overlay_ws = {}
_overlay_params_memo = {}


class OverlayFont:
    """The glyph atlas of ``draw_plates`` on a device, uploaded once: ``atlas`` uint8 [G, gh, gw] coverage and ``glyph_of`` uint16
    [8, 64] as ``yolov6.utils.overlay.build_atlas`` makes them (or any caller's data with the thirteen fixed glyphs)."""

    def __init__(self, atlas, glyph_of, device='cuda'):
        from yolov6.utils.overlay import check_font
        self.atlas_np, self.glyph_of_np = check_font(atlas, glyph_of)
        self.device = _cuda_device(device, 'OverlayFont lives on a GPU; the CPU path takes the arrays themselves (draw_plates_np)')
        self.atlas = torch.from_numpy(self.atlas_np).to(self.device)
        self.glyph_of = torch.from_numpy(self.glyph_of_np.view(np.int16)).to(self.device)      # the bits of the uint16 table
        self.n_glyphs, self.gh, self.gw = self.atlas_np.shape


def _overlay_params(font, styles, palette, matrix, show_id, label, draw_box):
    """lp_overlay_params of checked styles and palette, the colours in the bytes of a frame of ``matrix`` (None: BGR)."""
    from yolov6.utils.redact import fill_bytes
    key = (font.n_glyphs, font.gh, font.gw, tuple(styles), None if palette is None else palette.tobytes(), matrix, bool(show_id),
           bool(label), bool(draw_box))
    p = _overlay_params_memo.get(key)       # the colour conversion of an NV12 matrix is not free: once per distinct call
    if p is not None:
        return p
    if len(_overlay_params_memo) >= 64:
        _overlay_params_memo.clear()
    p = _overlay_params_memo[key] = abi.OverlayParams()
    p.n_styles = len(styles)
    for d, s in zip(p.styles, styles):
        for name in ('box', 'quad', 'plate', 'text'):
            getattr(d, name)[:] = fill_bytes(getattr(s, name), matrix)
        d.t, d.a_line, d.a_plate, d.a_text, d.pad = s.t, s.a_line, s.a_plate, s.a_text, s.pad
    p.n_palette = 0 if palette is None else len(palette)
    for k in range(p.n_palette):
        p.palette[k][:] = fill_bytes(tuple(int(v) for v in palette[k]), matrix)
    p.n_glyphs, p.gh, p.gw = font.n_glyphs, font.gh, font.gw
    p.show_id, p.label, p.draw_box = int(bool(show_id)), int(bool(label)), int(bool(draw_box))
    return p


def draw_plates(frames, det, count, atlas, glyph_of=None, tid=None, style=None, styles=None, palette=None, show_id=True, label=True,
                draw_box=True, status=None):
    """Draw the detections of B device frames onto them IN PLACE (lp_overlay_draw_batch, two launches per 64 frames on the current
    stream, no host read): box outline, corner-quad outline and a label with the track id and the eight heads' characters.
    ``frames`` is a list of contiguous uint8 CUDA [h,w,3] BGR tensors or of ``Nv12Frame`` with CUDA planes (one kind; NV12 is drawn
    in its own planes, no BGR copy exists); ``det`` [>= B,max_det,28] + ``count`` int32 on the device exactly as
    ``detect_frames_padded``, ``detect_tiled_padded``, ``TileGate.detect_padded``, ``PlateTracker.update`` (det_out) or the
    tracker's ``last_hold`` leave them; ``tid`` int32 [>= B,max_det] as ``PlateTracker.update`` returns it, or None; ``style`` int32
    [>= B,max_det] picks one of ``styles`` (a list of up to 8 ``yolov6.utils.overlay.Style``, colours (B, G, R), converted with
    the frame's matrix for NV12) per row, < 0 skips the row; ``palette`` uint8 [P <= 64, 3] colours the quad and the label plate
    by ``tid % P``.  ``atlas`` is an ``OverlayFont`` (uploaded once, reused), or the two arrays of one.  Writes into the caller's
    tensors and returns status [B,max_det] int32: 1 = corners, 2 = box, 3 = nothing drawable, 0 = no such row or a skipped one.
    ``yolov6.utils.overlay.draw_plates_np`` is the same computation on the CPU, byte for byte.

    THE OVERLAY GOES LAST on a stream: crops and best shots read the frames first, ``redact_plates`` comes next, then this call, so
    outlines sit on top of a mosaic.  Draw on a clone when other consumers need the clean frame."""
    from yolov6.utils.overlay import check_palette, check_styles
    if not frames:
        raise ValueError('draw_plates needs at least one frame')
    dev, nv12 = _frames_on(frames, 'draw_plates')
    _check_det_count(det, count, min_batch=len(frames))
    if det.device != dev or det.shape[1] < 1:
        raise ValueError('det must be on the frames\' device with max_det >= 1')
    font = atlas if isinstance(atlas, OverlayFont) else OverlayFont(atlas, glyph_of, dev)
    if font.device != dev:
        raise ValueError('the OverlayFont is on %s, the frames on %s' % (font.device, dev))
    styles, palette = check_styles(styles), check_palette(palette)
    n, max_det = len(frames), det.shape[1]
    for name, a in (('tid', tid), ('style', style)):
        if a is not None and not (a.is_cuda and a.device == dev and a.dtype == torch.int32 and a.dim() == 2 and a.shape[0] >= n
                                  and a.shape[1] == max_det and a.is_contiguous()):
            raise ValueError('%s must be a contiguous CUDA int32 [>= %d, %d] tensor on the frames\' device' % (name, n, max_det))
    status = _buffer(status, (n, max_det), torch.int32, dev, 'status')
    desc = _plane_descs(abi.RedactDesc, frames, nv12)
    # one call per run of frames that share the colours' bytes: a BGR list is one run, an NV12 list one per matrix
    key = [f.matrix if nv12 else None for f in frames]
    lib = abi.load()
    with torch.cuda.device(dev):
        for b0, b1 in _runs_by_key(key):
            params = _overlay_params(font, styles, palette, key[b0], show_id, label, draw_box)
            run = _desc_run(desc, b0)
            need = lib.lp_overlay_workspace_bytes(b1 - b0, max_det)
            ws = _stream_workspace(_overlay_ws, dev, need)
            abi.check(lib.lp_overlay_draw_batch(run, b1 - b0, _dptr(det[b0:b1]), _dptr(count[b0:b1]), max_det,
                                                None if tid is None else _dptr(tid[b0:b1]), None if style is None else _dptr(style[b0:b1]),
                                                ctypes.byref(params), _dptr(font.atlas), _dptr(font.glyph_of), _dptr(status[b0:b1]),
                                                _aligned(ws), need, _stream_ptr(dev)), 'lp_overlay_draw_batch')
    return status
